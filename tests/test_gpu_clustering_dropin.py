"""`usearch_clustering` / `usearch_clustering_members` through the drop-in `libusearch_c.so` (include/usearch_c_dropin.h), driven as
tests/test_gpu_compact_dropin.py drives the library, and `cluster(begin, end, config, keys, distances)` through the C++ class
surface (tests/cpp/cluster_surface.cpp). What they return is held against the model of tests/cluster_model.py fed by
`Index.cluster(vectors, level)` and `Index.distances` over the same image."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import usearch_amd
from tests import util
from tests.cluster_feeds import DeviceFeed
from tests.test_gpu_dropin import METRIC, SCALAR, Options, lib, ok, ptr  # noqa: F401  (`lib` is the module's fixture)

pytestmark = pytest.mark.gpu

NDIM = 33


@pytest.fixture()
def clustering(lib):  # noqa: F811
    err = C.POINTER(C.c_char_p)
    lib.usearch_clustering.restype = None
    lib.usearch_clustering.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p,
                                       C.c_void_p, C.c_void_p, err]
    lib.usearch_clustering_members.restype = None
    lib.usearch_clustering_members.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p,
                                               C.c_void_p, err]
    return lib


def by_vectors(lib, index, queries, min_count, max_count):  # noqa: F811
    keys, distances = np.zeros(len(queries), dtype=np.uint64), np.zeros(len(queries), dtype=np.float32)
    stats, err = np.zeros(3, dtype=np.uint64), C.c_char_p()
    lib.usearch_clustering(index, ptr(queries), SCALAR["i8"], len(queries), queries.strides[0], min_count, max_count, ptr(keys),
                           ptr(distances), ptr(stats), C.byref(err))
    return keys, distances, stats, err.value


def by_keys(lib, index, members, count, min_count, max_count):  # noqa: F811
    keys, distances = np.zeros(count, dtype=np.uint64), np.zeros(count, dtype=np.float32)
    stats, err = np.zeros(3, dtype=np.uint64), C.c_char_p()
    lib.usearch_clustering_members(index, ptr(members) if members is not None else None, count, min_count, max_count, ptr(keys),
                                   ptr(distances), ptr(stats), C.byref(err))
    return keys, distances, stats, err.value


def assert_same(got, model):
    keys, distances, stats, error = got
    assert not error, error
    assert np.array_equal(keys, model["keys"]) and util.same_float_bits(distances, model["distances"])
    assert stats.tolist() == [model["clusters"], model["visited_members"], model["computed_distances"]]


def saved(lib, index) -> np.ndarray:  # noqa: F811
    err = C.c_char_p()
    image = np.zeros(lib.usearch_serialized_length(index, C.byref(err)), dtype=np.uint8)
    ok(err)
    lib.usearch_save_buffer(index, ptr(image), image.size, C.byref(err))
    ok(err)
    return image


def test_a_loaded_image_clusters_like_the_model(clustering, reference):
    lib = clustering  # noqa: F811
    err = C.c_char_p()
    image, vectors, _ = util.build_image(2000, NDIM, "l2sq", "i8", seed=11, connectivity=4)
    index = lib.usearch_init(None, C.byref(err))
    ok(err)
    lib.usearch_load_buffer(index, ptr(image), image.size, C.byref(err))
    ok(err)
    feed = DeviceFeed(usearch_amd.Index.restore(image, device=0), image, vectors, "i8")
    queries = util.make_vectors(500, NDIM, "i8", seed=21)
    assert_same(by_vectors(lib, index, queries, 6, 4), feed.run(queries, 6, 4))
    members = feed.facts.keys[np.random.default_rng(22).choice(2000, 300, replace=False)]
    assert_same(by_keys(lib, index, members, 300, 6, 4), feed.run_members(members, 6, 4))
    assert_same(by_keys(lib, index, None, 2000, 6, 4), feed.run_members(feed.facts.keys, 6, 4))
    assert by_keys(lib, index, np.array([5], dtype=np.uint64), 1, 6, 4)[3] == b"Key missing!"
    assert b"max_clusters" in by_vectors(lib, index, queries, 6, 0)[3]
    lib.usearch_free(index, C.byref(err))


def test_right_after_deferred_adds(clustering):
    """`usearch_add` defers the linking of a batch: a clustering call links it first, as a search does. The model runs over the image
    saved afterwards."""
    lib = clustering  # noqa: F811
    err = C.c_char_p()
    vectors = util.make_vectors(900, NDIM, "i8", seed=31)
    options = Options(METRIC["l2sq"], None, SCALAR["i8"], NDIM, 4, 64, 64, False)
    index = lib.usearch_init(C.byref(options), C.byref(err))
    ok(err)
    lib.usearch_reserve(index, 900, C.byref(err))
    for i in range(900):
        lib.usearch_add(index, 5000 + i, ptr(vectors[i]), SCALAR["i8"], C.byref(err))
        ok(err)
    queries = util.make_vectors(200, NDIM, "i8", seed=32)
    got = by_vectors(lib, index, queries, 5, 3)
    image = saved(lib, index)
    feed = DeviceFeed(usearch_amd.Index.restore(image, device=0), image, vectors, "i8")
    assert feed.facts.max_level >= 2 and np.array_equal(feed.facts.keys, 5000 + np.arange(900, dtype=np.uint64))
    assert_same(got, feed.run(queries, 5, 3))
    assert_same(by_keys(lib, index, None, 900, 5, 3), feed.run_members(feed.facts.keys, 5, 3))
    lib.usearch_free(index, C.byref(err))


def test_the_class_surface_clusters_like_the_model(tmp_path, reference):
    from tests.test_cluster_model import build_cluster_surface
    binary = build_cluster_surface(tmp_path)
    image, vectors, _ = util.build_image(2000, NDIM, "l2sq", "i8", seed=11, connectivity=4)
    queries = util.make_vectors(400, NDIM, "i8", seed=41)
    image_path, queries_path, out_path = (os.path.join(str(tmp_path), name) for name in ("image.usearch", "Q.bin", "out.bin"))
    image.tofile(image_path), queries.tofile(queries_path)
    out = subprocess.run([binary, "run", image_path, queries_path, "400", str(NDIM), "6", "4", out_path], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    raw = np.fromfile(out_path, dtype=np.uint8)
    record = 400 * 12 + 24
    assert raw.size == 2 * record
    feed = DeviceFeed(usearch_amd.Index.restore(image, device=0), image, vectors, "i8")
    for part, model in ((raw[:record], feed.run(queries, 6, 4)), (raw[record:], feed.run_members(1000 + np.arange(400, dtype=np.uint64), 6, 4))):
        got = (part[:3200].view(np.uint64), part[3200:4800].view(np.float32), part[4800:].view(np.uint64), None)
        assert_same(got, model)
