"""GPU: the three routes of exact search (the wave kernel, the matrix-unit tile, the screened route) through the three ways in — an
index with host buffers (`Index.search(exact=…)`), an index with device pointers (`Index.exact_search_device`) and a raw dataset
(`usearch_amd.exact_search`). All of them settle the route in one place (csrc/engine.hip, `exact_search_routed`): whichever way a
route is asked for, it returns the same bits. 70 queries end inside a tile of 64, 700 rows end inside a row tile."""
import functools

import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu
ROWS, NDIM, QUERIES, K = 700, 64, 70, 10
ROUTES = {"wave": (True, False), "tiled": ("tiled", True), "screened": ("screened", "screened")}  # name → (`exact=`, `tiled=`)


@functools.lru_cache(maxsize=None)
def results(route):
    """→ {way in: (keys, distances, counts or None)} of `route` for the one seeded case, computed once."""
    import torch
    import usearch_amd
    image, vectors, _ = util.build_image(ROWS, NDIM, "cos", "f32", seed=191, clustered=False, connectivity=4, expansion_add=16,
                                         keys=np.arange(ROWS, dtype=np.uint64))
    queries = util.make_vectors(QUERIES, NDIM, "f32", seed=192, clustered=False)
    exact, tiled = ROUTES[route]
    index = usearch_amd.Index.restore(image)
    host = index.search(queries, K, exact=exact)
    device = torch.device("cuda", 0)
    held = torch.from_numpy(queries).to(device)
    keys = torch.zeros((QUERIES, K), dtype=torch.int64, device=device)
    distances = torch.zeros((QUERIES, K), dtype=torch.float32, device=device)
    counts = torch.zeros(QUERIES, dtype=torch.int64, device=device)
    torch.cuda.synchronize()
    index.exact_search_device(held.data_ptr(), QUERIES, held.stride(0) * 4, K, keys.data_ptr(), distances.data_ptr(), counts.data_ptr(),
                              tiled=tiled)
    torch.cuda.synchronize()
    raw_keys, raw_distances = usearch_amd.exact_search(vectors, queries, K, metric="cos", tiled=tiled)
    return {"host": (host.keys, host.distances, host.counts),
            "device": (keys.cpu().numpy().view(np.uint64), distances.cpu().numpy(), counts.cpu().numpy().view(np.uint64)),
            "dataset": (raw_keys, raw_distances, None)}


def assert_same(a, b):
    assert np.array_equal(a[0], b[0]), "other keys"
    assert util.same_float_bits(a[1], b[1]), "other distance bits"
    if a[2] is not None and b[2] is not None:
        assert np.array_equal(a[2], b[2]), "other counts"


@pytest.mark.parametrize("route", list(ROUTES))
def test_a_route_returns_the_same_bits_whichever_way_it_is_reached(reference, route):
    got = results(route)
    assert (got["host"][2] == K).all() and (got["host"][0] < ROWS).all()
    assert_same(got["host"], got["device"])
    assert_same(got["host"], got["dataset"])


def test_the_screened_route_returns_the_wave_kernels_bits(reference):
    for way in ("host", "device", "dataset"):
        assert_same(results("screened")[way], results("wave")[way])
