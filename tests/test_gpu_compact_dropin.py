"""`usearch_isolate` / `usearch_compact` through the drop-in `libusearch_c.so` (include/usearch_c_dropin.h), driven as
tests/test_gpu_dropin.py drives the library, and `isolate()` / `compact()` through the C++ class surface
(tests/cpp/compact_surface.cpp: the reference's own `test_isolate` scenario, cpp/test.cpp:1147-1180)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import oraclebind, refbind
from tests import compact_model, util
from tests.test_gpu_dropin import METRIC, SCALAR, Options, lib, ok, ptr  # noqa: F401  (`lib` is the module's fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NDIM = 24


@pytest.fixture()
def compacting(lib):  # noqa: F811
    err = C.POINTER(C.c_char_p)
    for name in ("usearch_isolate", "usearch_compact"):
        getattr(lib, name).restype = C.c_size_t
        getattr(lib, name).argtypes = [C.c_void_p, err]
    return lib


def saved(lib, index) -> np.ndarray:  # noqa: F811
    err = C.c_char_p()
    image = np.zeros(lib.usearch_serialized_length(index, C.byref(err)), dtype=np.uint8)
    ok(err)
    lib.usearch_save_buffer(index, ptr(image), image.size, C.byref(err))
    ok(err)
    return image


def search_many(lib, index, queries, k, filter=None):  # noqa: F811
    keys = np.zeros((len(queries), k), dtype=np.uint64)
    distances = np.zeros((len(queries), k), dtype=np.float32)
    counts = np.zeros(len(queries), dtype=np.uint64)
    err = C.c_char_p()
    if filter is None:
        lib.usearch_search_many(index, ptr(queries), SCALAR["f32"], len(queries), queries.strides[0], k, ptr(keys), keys.strides[0],
                                ptr(distances), distances.strides[0], ptr(counts), None, None, C.byref(err))
    else:
        lib.usearch_filtered_search_many(index, filter, ptr(queries), SCALAR["f32"], len(queries), queries.strides[0], k, ptr(keys),
                                         keys.strides[0], ptr(distances), distances.strides[0], ptr(counts), None, None, C.byref(err))
    return keys, distances, counts, err.value


def check_sequence(lib, index, vectors, keys, removed_keys, capacity_for_more):  # noqa: F811
    """From "members removed" on: isolate, compact, and the index behaves as a fresh one of the survivors."""
    err = C.c_char_p()
    kept_keys = [int(key) for key in keys if int(key) not in set(removed_keys)]
    row_of = {int(key): vectors[i] for i, key in enumerate(keys)}
    stale = lib.usearch_filter_from_key_range(index, 0, 2**63, C.byref(err))
    ok(err)
    lists, levels, image_keys, entry, _ = compact_model.read_image(saved(lib, index))
    assert sum(key == compact_model.FREE_KEY for key in image_keys) == len(removed_keys)
    model = compact_model.compact(lists, levels, image_keys, entry)

    assert lib.usearch_isolate(index, C.byref(err)) == model["pruned_edges"]
    ok(err)
    assert lib.usearch_isolate(index, C.byref(err)) == 0
    assert lib.usearch_compact(index, C.byref(err)) == len(removed_keys)
    ok(err)
    assert lib.usearch_compact(index, C.byref(err)) == 0, "nothing is left to drop"
    assert lib.usearch_size(index, C.byref(err)) == len(kept_keys)
    for key in removed_keys:
        assert not lib.usearch_contains(index, int(key), C.byref(err))
    row = np.zeros(NDIM, dtype=np.float32)
    for key in kept_keys:
        assert lib.usearch_contains(index, key, C.byref(err))
        assert lib.usearch_get(index, key, 1, ptr(row), SCALAR["f32"], C.byref(err)) == 1
        assert np.array_equal(row, row_of[key])
    image = saved(lib, index)
    got = compact_model.read_image(image)
    assert (got[0], got[1], got[2], got[3], got[4]) == (model["lists"], model["levels"], model["keys"], model["entry"], model["max_level"])

    # ten more: appended behind the survivors, nothing is recycled
    lib.usearch_reserve(index, capacity_for_more, C.byref(err))
    ok(err)
    more = util.make_vectors(10, NDIM, "f32", seed=99)
    for i in range(10):
        lib.usearch_add(index, 70000 + i, ptr(more[i]), SCALAR["f32"], C.byref(err))
        ok(err)
    image = saved(lib, index)
    oracle = oraclebind.OracleIndex(image)
    assert len(oracle) == len(kept_keys) + 10
    assert [oracle.key(len(kept_keys) + i) for i in range(10)] == [70000 + i for i in range(10)]
    assert [oracle.key(slot) for slot in range(len(kept_keys))] == kept_keys
    reference = refbind.RefIndex.from_buffer(image, dtype="f32")
    assert len(reference) == len(kept_keys) + 10
    queries = np.ascontiguousarray(np.stack([row_of[key] for key in kept_keys[:40]]))
    found, _, counts, error = search_many(lib, index, queries, 5)
    # (the walk is approximate and nobody relinked the lists that got short: nearly every stored row still finds itself first)
    assert not error and (found[:, 0] == np.array(kept_keys[:40], dtype=np.uint64)).mean() >= 0.9 and (counts == 5).all()
    rkeys = reference.search(queries, 5, dtype="f32", threads=1)[0]
    assert (found == rkeys).mean() > 0.9

    # a filter made before the compact describes the old numbering: refused; one made now works
    _, _, _, error = search_many(lib, index, queries, 5, filter=stale)
    assert error, "a filter made before the compact was accepted"
    fresh = lib.usearch_filter_from_key_range(index, kept_keys[0], kept_keys[0], C.byref(err))
    ok(err)
    found, _, counts, error = search_many(lib, index, queries, 5, filter=fresh)
    assert not error and (counts == 1).all() and (found[:, 0] == kept_keys[0]).all()
    lib.usearch_filter_free(stale, C.byref(err))
    lib.usearch_filter_free(fresh, C.byref(err))


def test_add_search_remove_isolate_compact(compacting):
    lib = compacting  # noqa: F811
    err = C.c_char_p()
    vectors = util.make_vectors(400, NDIM, "f32", seed=61)
    keys = np.arange(400) + 3000
    options = Options(METRIC["cos"], None, SCALAR["f32"], NDIM, 8, 64, 64, False)
    index = lib.usearch_init(C.byref(options), C.byref(err))
    ok(err)
    lib.usearch_reserve(index, 400, C.byref(err))
    for i in range(400):
        lib.usearch_add(index, int(keys[i]), ptr(vectors[i]), SCALAR["f32"], C.byref(err))
        ok(err)
    found, _, _, error = search_many(lib, index, np.ascontiguousarray(vectors[:20]), 5)
    assert not error and np.array_equal(found[:, 0], keys[:20].astype(np.uint64))
    removed = [int(key) for key in np.random.default_rng(62).choice(keys, 100, replace=False)]
    for key in removed:
        assert lib.usearch_remove(index, key, C.byref(err)) == 1
        ok(err)
    check_sequence(lib, index, vectors, keys, removed, 400)
    lib.usearch_free(index, C.byref(err))


def loaded_index(lib, seed):  # noqa: F811
    """An index that came from `usearch_load_buffer` of a reference-built image with removed keys; nothing else has touched it."""
    err = C.c_char_p()
    keys = np.arange(400) + 3000
    removed = [int(key) for key in np.random.default_rng(seed).choice(keys, 100, replace=False)]
    image, vectors, _ = util.build_image(400, NDIM, "cos", "f32", seed=seed + 1, connectivity=8, keys=keys.astype(np.uint64), remove=removed)
    index = lib.usearch_init(None, C.byref(err))
    ok(err)
    lib.usearch_load_buffer(index, ptr(image), image.size, C.byref(err))
    ok(err)
    assert lib.usearch_size(index, C.byref(err)) == 300
    return index, image, vectors, keys, removed


def test_a_loaded_image_with_removed_members_goes_through_the_same_sequence(compacting, reference):
    """The image's own graph is isolated and compacted (the model applied to the loaded image, list for list): nothing is linked
    anew on the way."""
    lib = compacting  # noqa: F811
    err = C.c_char_p()
    index, image, vectors, keys, removed = loaded_index(lib, 63)
    check_sequence(lib, index, vectors, keys, removed, 400)
    lib.usearch_free(index, C.byref(err))


def test_a_loaded_image_compacts_without_an_isolate_first(compacting, reference):
    lib = compacting  # noqa: F811
    err = C.c_char_p()
    index, image, vectors, keys, removed = loaded_index(lib, 65)
    lists, levels, image_keys, entry, _ = compact_model.read_image(image)
    model = compact_model.compact(lists, levels, image_keys, entry)
    assert lib.usearch_compact(index, C.byref(err)) == 100
    ok(err)
    got = compact_model.read_image(saved(lib, index))
    assert (got[0], got[1], got[2], got[3], got[4]) == (model["lists"], model["levels"], model["keys"], model["entry"], model["max_level"])
    lib.usearch_free(index, C.byref(err))


def test_an_isolate_of_a_loaded_image_is_saved_and_survives_the_next_mutation(compacting, reference):
    lib = compacting  # noqa: F811
    err = C.c_char_p()
    index, image, vectors, keys, removed = loaded_index(lib, 67)
    lists, levels, image_keys, entry, max_level = compact_model.read_image(image)
    expected, erased = compact_model.isolate(lists, image_keys)
    assert erased > 0
    assert lib.usearch_isolate(index, C.byref(err)) == erased
    ok(err)
    got = compact_model.read_image(saved(lib, index))
    assert (got[0], got[1], got[2], got[3], got[4]) == (expected, levels, image_keys, entry, max_level)
    # a rename touches no list: the isolated lists are still what is saved
    kept = int(next(key for key in keys if int(key) not in set(removed)))
    assert lib.usearch_rename(index, kept, 99999, C.byref(err)) == 1
    ok(err)
    renamed = [99999 if key == kept else key for key in image_keys]
    got = compact_model.read_image(saved(lib, index))
    assert (got[0], got[1], got[2], got[3], got[4]) == (expected, levels, renamed, entry, max_level)
    assert lib.usearch_isolate(index, C.byref(err)) == 0
    lib.usearch_free(index, C.byref(err))


def test_the_class_surface_runs_the_references_isolate_scenario(tmp_path):
    from tests.test_compact_exports import build_compact_surface
    binary = build_compact_surface(tmp_path)
    out = subprocess.run([binary, "run"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
