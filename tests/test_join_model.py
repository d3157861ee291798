"""CPU: the facts the device's semantic join rests on (usearch_amd/csrc/join.hip), checked against the compiled reference and
the oracle — the prefix property of one search per man, the order independence of deferred acceptance, the model fed by the
reference against the model fed by the oracle in the kernels' layout, the symmetry of the husband's distance — and the ctypes
mirrors of the join's structs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import oraclebind, refbind
from tests import join_model, util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_reference = pytest.mark.skipif(not refbind.available(), reason="oracle/_ref is built by build() where the reference is mounted")


def _prefix_index(metric, dtype, ndim=24, n=1500, seed=5):
    image, vectors, index = util.build_image(n, ndim, metric, dtype, seed=seed)
    queries = util.make_vectors(60, ndim, dtype, seed=seed + 1)
    return index, queries


@needs_reference
@pytest.mark.parametrize("metric,dtype", [("cos", "f32"), ("l2sq", "f16"), ("ip", "f32")])
@pytest.mark.parametrize("exact", [False, True])
def test_search_k_is_a_prefix_of_search_with_more_up_to_expansion(metric, dtype, exact):
    """index.hpp:3049-3068: the beam runs with ef = max(expansion, k) and keeps k, so search(k = i) is the first i rows of
    search(k = expansion) for every i <= expansion — one search per man gives his whole list."""
    index, queries = _prefix_index(metric, dtype)
    expansion = 12
    index.expansion_search = expansion
    keys, distances, counts = index.search(queries, expansion, exact=exact)[:3]
    for i in range(1, expansion + 1):
        k_i, d_i, c_i = index.search(queries, i, exact=exact)[:3]
        assert np.array_equal(c_i, np.minimum(counts, i))
        assert np.array_equal(k_i, keys[:, :i]), f"search(k={i}) is not a prefix"
        assert util.same_float_bits(d_i, distances[:, :i])


@needs_reference
@pytest.mark.parametrize("metric,dtype", [("cos", "f32"), ("l2sq", "f16"), ("ip", "f32")])
def test_search_beyond_expansion_is_not_a_prefix(metric, dtype):
    """… and beyond `expansion` the beam widens with k, so the first rows change: why proposals past ef need searches of their own."""
    index, queries = _prefix_index(metric, dtype, ndim=48, n=3000, seed=9)
    expansion = 2
    index.expansion_search = expansion
    narrow = index.search(queries, expansion)[0]
    wide = index.search(queries, 24)[0]
    assert (wide[:, :expansion] != narrow).any(), "a wider beam found nothing nearer: the data is too easy to show it"


def _exact_lists(n_men, n_women, seed):
    rng = np.random.default_rng(seed)
    men, women = rng.standard_normal((n_men, 8)), rng.standard_normal((n_women, 8))
    d = ((men[:, None, :] - women[None, :, :]) ** 2).sum(-1)  # float64: tie-free
    order = np.argsort(d, axis=1)
    search = lambda m, k: [(int(w), float(d[m, w])) for w in order[m, :k]]
    distance = lambda w, m: float(d[m, w])
    return search, distance


@pytest.mark.parametrize("n_men,n_women,p", [(200, 300, 5), (300, 300, 0), (150, 120, 4)])
def test_the_matching_does_not_depend_on_the_order_of_proposals(n_men, n_women, p):
    """Man-proposing deferred acceptance with strict, truncated preferences ends in one man-optimal stable matching whatever the
    order of proposals: FIFO, the queue reversed and three seeded random orders agree — what lets every free man propose at once."""
    search, distance = _exact_lists(n_men, n_women, seed=n_men + n_women)
    p = join_model.default_max_proposals(n_men, p)
    fifo = join_model.stable_marriage(n_men, search, distance, p)
    assert fifo, "nobody matched"
    assert join_model.stable_marriage(n_men, search, distance, p, order="reversed") == fifo
    for seed in (1, 2, 3):
        assert join_model.stable_marriage(n_men, search, distance, p, order="random", seed=seed) == fifo


def test_default_max_proposals_follows_the_reference():
    assert join_model.default_max_proposals(1000) == int(np.log(1000) + 1) == 7
    assert join_model.default_max_proposals(1000, threads=16) == 22
    assert join_model.default_max_proposals(5, 100) == 5
    assert join_model.default_max_proposals(10**6, 12) == 12


def _case_images(case):
    metric, dtype, ndim, n_a, n_b, p, expansion, exact = case
    image_a, vectors_a, ref_a = util.build_image(n_a, ndim, metric, dtype, seed=join_model.SEED_A,
                                                 keys=np.arange(n_a, dtype=np.uint64) + join_model.KEYS_A)
    image_b, vectors_b, ref_b = util.build_image(n_b, ndim, metric, dtype, seed=join_model.SEED_B,
                                                 keys=np.arange(n_b, dtype=np.uint64) + join_model.KEYS_B)
    return image_a, vectors_a, ref_a, image_b, vectors_b, ref_b


def model_with(search_in, vectors_a, vectors_b, case, lanes):
    """The model of `join(a, b)` fed by `search_in(side, query_row, k)` → (slots, distances) and the oracle's distance."""
    metric, dtype, ndim, n_a, n_b, p, expansion, exact = case

    def searcher(side, rows):
        return lambda m, k: list(zip(*search_in(side, rows[m], k)))

    distance = lambda first, second: lambda w, m: oraclebind.distance(first[w], second[m], metric, dtype, ndim, lanes)
    return join_model.join(n_a, n_b, searcher("b", vectors_a), searcher("a", vectors_b), distance(vectors_b, vectors_a),
                           distance(vectors_a, vectors_b), max_proposals=p)


def oracle_searcher(image_a, image_b, case, lanes, frontier_in_top):
    metric, dtype, ndim, n_a, n_b, p, expansion, exact = case
    oracles = {"a": (oraclebind.OracleIndex(image_a), join_model.KEYS_A), "b": (oraclebind.OracleIndex(image_b), join_model.KEYS_B)}

    def search(side, row, k):
        oracle, base = oracles[side]
        keys, distances, counts = oracle.search(row[None, :], k, dtype=dtype, expansion=expansion, exact=exact, lanes=lanes,
                                                frontier_in_top=frontier_in_top)[:3]
        found = int(counts[0])
        return [int(x) - base for x in keys[0, :found]], [float(x) for x in distances[0, :found]]
    return search


@needs_reference
@pytest.mark.parametrize("case", join_model.CASES, ids=[f"{c[0]}-{c[1]}-{c[3]}x{c[4]}-P{c[5]}-ef{c[6]}{'-exact' if c[7] else ''}"
                                                        for c in join_model.CASES])
def test_model_fed_by_the_reference_equals_model_fed_by_the_oracle(case):
    """The model run on the reference's own search (refbind) and on the oracle in the kernels' summation layout (both frontiers)
    give the same matching on the seeds the GPU tests use: the GPU, equal to the second, is thereby equal to the first."""
    metric, dtype, ndim, n_a, n_b, p, expansion, exact = case
    image_a, vectors_a, ref_a, image_b, vectors_b, ref_b = _case_images(case)
    refs = {"a": (ref_a, join_model.KEYS_A), "b": (ref_b, join_model.KEYS_B)}
    for ref, _ in refs.values():
        ref.expansion_search = expansion

    def reference_search(side, row, k):
        ref, base = refs[side]
        keys, distances, counts = ref.search(row[None, :], k, exact=exact)[:3]
        found = int(counts[0])
        return [int(x) - base for x in keys[0, :found]], [float(x) for x in distances[0, :found]]

    lanes = join_model.lanes_per_row(dtype, ndim)
    reference = model_with(reference_search, vectors_a, vectors_b, case, lanes)
    assert len(reference) > 0.2 * min(n_a, n_b)
    for frontier_in_top in (False, True):
        assert model_with(oracle_searcher(image_a, image_b, case, lanes, frontier_in_top), vectors_a, vectors_b, case,
                          lanes) == reference, f"frontier_in_top={frontier_in_top}"


SYMMETRY_CASES = join_model.CASES + [("l2sq", "i8", 32, 400, 500, 6, 64, False), ("hamming", "b1", 64, 400, 500, 6, 64, False)]


@pytest.mark.parametrize("case", SYMMETRY_CASES, ids=[f"{c[0]}-{c[1]}-{c[3]}x{c[4]}{'-exact' if c[7] else ''}" for c in SYMMETRY_CASES])
def test_the_husband_distance_is_symmetric_bit_for_bit(case):
    """The device keeps the winning proposal's own d(man, woman); the reference recomputes d(woman, man) (index.hpp:4497-4498).
    For every pair in the lists of the GPU tests' joins the two are the same float."""
    metric, dtype, ndim, n_a, n_b, p, expansion, exact = case
    image_a, vectors_a, _, image_b, vectors_b, _ = _case_images(case)
    lanes = join_model.lanes_per_row(dtype, ndim)
    search = oracle_searcher(image_a, image_b, case, lanes, frontier_in_top=False)
    men, women, side = (vectors_a, vectors_b, "b") if n_a <= n_b else (vectors_b, vectors_a, "a")
    width = max(p, join_model.default_max_proposals(len(men), p))
    checked = 0
    for m in range(len(men)):
        for w in search(side, men[m], width)[0]:
            forward = oraclebind.distance(men[m], women[w], metric, dtype, ndim, lanes)
            backward = oraclebind.distance(women[w], men[m], metric, dtype, ndim, lanes)
            assert np.float32(forward).view(np.uint32) == np.float32(backward).view(np.uint32), (m, w, forward, backward)
            checked += 1
    assert checked > len(men)


def test_join_ctypes_mirrors_follow_the_header_field_by_field():
    """The join's config and stats structs of include/usearch_amd.h against their ctypes mirrors, name by name, type by type."""
    from usearch_amd import index as host
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "usearch_amd.h")).read(), flags=re.S)
    ctype = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double}
    for c_name, mirror in (("usearch_amd_join_config_t", host.JoinConfig), ("usearch_amd_join_stats_t", host.JoinStats)):
        found = re.search(r"typedef struct " + c_name + r"\s*\{(.*?)\}\s*" + c_name + r"\s*;", header, flags=re.S)
        assert found, c_name
        declared = []
        for kind, names in re.findall(r"^\s*(\w+)\s+(\w+(?:\s*,\s*\w+)*)\s*;", found.group(1), flags=re.M):
            declared += [(name.strip(), ctype[kind]) for name in names.split(",")]
        assert [(name, kind) for name, kind in mirror._fields_] == declared, f"{c_name} and its ctypes mirror differ"
    assert "usearch_amd_join" in host.EXPORTED_SYMBOLS


def build_join_surface(directory) -> str:
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "usearch_amd", "lib")
    binary = os.path.join(str(directory), "usearch_amd_join_surface")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "join_surface.cpp"), "-L", lib, "-l:libusearch_c.so", f"-Wl,-rpath,{lib}",
                           "-o", binary])
    return binary


def test_the_cpp_join_caller_compiles_against_the_class_surface(tmp_path):
    """cpp/bench.cpp's join call — the free `join` with raw key arrays — and the member `join` with `unordered_map`s compile and link
    against include/usearch/index_dense.hpp (run on the device by tests/test_gpu_join.py)."""
    import subprocess
    binary = build_join_surface(tmp_path)
    assert "join through index_dense_t" in subprocess.check_output([binary, "link"]).decode()
