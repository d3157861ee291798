"""GPU: semantic join (`Index.join`, `usearch_amd_join`; usearch_amd/csrc/join.hip) against the literal model of the reference's
loop (tests/join_model.py) fed by the oracle in the kernels' layout — bit-exact to the device's own lists — plus the cases with
ties, removals, refusals and one join at scale."""
import numpy as np
import pytest

from oracle import oraclebind
from tests import join_model, util
from tests.test_join_model import build_join_surface, model_with, oracle_searcher

pytestmark = pytest.mark.gpu


def _restore(case, remove_a=(), remove_b=()):
    from usearch_amd import Index
    metric, dtype, ndim, n_a, n_b, p, expansion, exact = case
    image_a, vectors_a, _ = util.build_image(n_a, ndim, metric, dtype, seed=join_model.SEED_A,
                                             keys=np.arange(n_a, dtype=np.uint64) + join_model.KEYS_A, remove=remove_a)
    image_b, vectors_b, _ = util.build_image(n_b, ndim, metric, dtype, seed=join_model.SEED_B,
                                             keys=np.arange(n_b, dtype=np.uint64) + join_model.KEYS_B, remove=remove_b)
    return image_a, vectors_a, Index.restore(image_a), image_b, vectors_b, Index.restore(image_b)


@pytest.mark.parametrize("case", join_model.CASES, ids=[f"{c[0]}-{c[1]}-{c[3]}x{c[4]}-P{c[5]}-ef{c[6]}{'-exact' if c[7] else ''}"
                                                        for c in join_model.CASES])
def test_join_equals_the_model_of_the_reference_loop(case):
    metric, dtype, ndim, n_a, n_b, p, expansion, exact = case
    image_a, vectors_a, a, image_b, vectors_b, b = _restore(case)
    got = a.join(b, max_proposals=p, exact=exact, expansion=expansion)
    stats = a.join_stats()
    assert stats["a_proposes"] == (0 if n_b < n_a else 1)
    assert stats["max_proposals"] == join_model.default_max_proposals(min(n_a, n_b), p)
    if p > expansion and not exact:
        assert stats["lazy_searches"] > 0, "the proposals beyond expansion never ran"
    lanes = a.lanes_per_row
    model = model_with(oracle_searcher(image_a, image_b, case, lanes, frontier_in_top=stats["frontier"] == 2), vectors_a, vectors_b,
                       case, lanes)
    expected = {k + join_model.KEYS_A: v + join_model.KEYS_B for k, v in model.items()}
    assert got == expected
    assert stats["pairs"] == len(got) and stats["rounds"] >= 1 and stats["proposals"] >= len(got)
    assert len(set(got.values())) == len(got)
    # the pairs come in ascending order of a's slots
    keys_a, keys_b, _ = a.join_arrays(b, max_proposals=p, exact=exact, expansion=expansion)
    assert np.all(np.diff(keys_a.astype(np.int64)) > 0) and dict(zip(keys_a.tolist(), keys_b.tolist())) == got


@pytest.mark.parametrize("metric,dtype,ndim", [("l2sq", "i8", 32), ("hamming", "b1", 64)])
def test_join_with_ties_is_deterministic_one_to_one_and_weakly_stable(metric, dtype, ndim):
    case = (metric, dtype, ndim, 400, 500, 6, 64, False)
    image_a, vectors_a, a, image_b, vectors_b, b = _restore(case)
    first = a.join(b, max_proposals=6)
    frontier = a.join_stats()["frontier"]
    assert a.join(b, max_proposals=6) == first
    assert len(set(first.values())) == len(first) and first
    lanes = a.lanes_per_row
    search = oracle_searcher(image_a, image_b, case, lanes, frontier_in_top=frontier == 2)
    lists = {m: list(zip(*search("b", vectors_a[m], 6))) for m in range(len(vectors_a))}
    matching = {k - join_model.KEYS_A: v - join_model.KEYS_B for k, v in first.items()}
    for man, woman in matching.items():
        assert woman in [w for w, _ in lists[man]], f"man {man} married outside his list"
    distance = lambda w, m: oraclebind.distance(vectors_b[w], vectors_a[m], metric, dtype, ndim, lanes)
    assert join_model.weakly_stable(matching, lists, distance) == []


def test_removed_members_take_no_part():
    """Removed members are tombstones in the image (the reference writes the free key into their slots): no output key may be the
    free key, every output key is a live member, and the matching is the model's with tombstoned men not proposing and tombstoned
    women absent from every list (the oracle's search skips them as the reference's does)."""
    case = ("cos", "f32", 32, 400, 500, 6, 64, False)
    removed_a = np.arange(0, 400, 7) + join_model.KEYS_A
    removed_b = np.arange(3, 500, 5) + join_model.KEYS_B
    image_a, vectors_a, a, image_b, vectors_b, b = _restore(case, remove_a=removed_a, remove_b=removed_b)
    live_a = set((np.arange(400) + join_model.KEYS_A).tolist()) - set(removed_a.tolist())
    live_b = set((np.arange(500) + join_model.KEYS_B).tolist()) - set(removed_b.tolist())
    free_key = 2**64 - 1
    lanes = a.lanes_per_row
    for exact in (False, True):
        got = a.join(b, max_proposals=6, exact=exact)
        stats = a.join_stats()
        assert got and free_key not in got and free_key not in got.values()
        assert set(got) <= live_a and set(got.values()) <= live_b
        this_case = case[:7] + (exact,)
        search = oracle_searcher(image_a, image_b, this_case, lanes, frontier_in_top=stats["frontier"] == 2)
        distance = lambda w, m: oraclebind.distance(vectors_b[w], vectors_a[m], "cos", "f32", 32, lanes)
        model = join_model.join(400, 500, lambda m, k: list(zip(*search("b", vectors_a[m], k))), None, distance, None,
                                max_proposals=6, proposers_a=sorted(k - join_model.KEYS_A for k in live_a))
        assert got == {m + join_model.KEYS_A: w + join_model.KEYS_B for m, w in model.items()}


def test_refusals_are_named():
    from usearch_amd import Index
    case = ("cos", "f32", 32, 300, 300, 0, 64, False)
    image_a, _, a, _, _, b = _restore(case)
    with pytest.raises(RuntimeError, match="Can't join with itself, consider copying"):
        a.join(a)
    image_l2, _, _ = util.build_image(300, 32, "l2sq", "f32", seed=3)
    with pytest.raises(RuntimeError, match="different metrics, scalar kinds or dimensions"):
        a.join(Index.restore(image_l2))
    image_16, _, _ = util.build_image(300, 16, "cos", "f32", seed=3)
    with pytest.raises(RuntimeError, match="different metrics, scalar kinds or dimensions"):
        a.join(Index.restore(image_16))
    # P is capped at the proposers' size first (index.hpp:4394): only a side of more than 65535 members can ask for more
    import usearch_amd
    vectors = util.make_vectors(70000, 8, "f32", seed=4, clustered=False)
    big_a = Index.restore(usearch_amd.build(vectors, "l2sq", "f32").save_buffer())
    big_b = Index.restore(usearch_amd.build(vectors, "l2sq", "f32").save_buffer())
    with pytest.raises(RuntimeError, match="65535"):
        big_a.join(big_b, max_proposals=65536)


def test_join_at_scale_matches_a_copy_of_itself():
    """1M × 96 f32 cos joined with a second snapshot of the same image (cpp/bench.cpp:412-445): exact lists give the identity on
    tie-free data; HNSW lists give recall_join at least the index's own recall@1 at that expansion."""
    import usearch_amd
    from usearch_amd import Index
    n, ndim, expansion = 1_000_000, 96, 64
    vectors = np.random.default_rng(11).standard_normal((n, ndim)).astype(np.float32)
    image = usearch_amd.build(vectors, "cos", "f32").save_buffer()
    a, b = Index.restore(image), Index.restore(image)
    keys = np.arange(n, dtype=np.uint64)
    a_keys, b_keys, stats = a.join_arrays(b, expansion=expansion)
    recall_join = float(np.mean(a_keys == b_keys)) * len(a_keys) / n
    # every man whose nearest find is himself proposes to himself first and wins: the lists are the same walk (prefix property)
    recall_at_1 = float(np.mean(a.search(vectors, 1, expansion=expansion).keys[:, 0] == keys))
    assert recall_join >= recall_at_1, (recall_join, recall_at_1, stats.as_dict())
    assert len(set(b_keys.tolist())) == len(b_keys)
    # weakly stable on a sample of men, under the device's own lists (P entries at that expansion)
    men = np.random.default_rng(13).choice(n, 2000, replace=False)
    assert _weakly_stable_sample(a, b, vectors, a_keys, b_keys, men, int(stats.max_proposals), expansion) == []
    a_keys, b_keys, _ = a.join_arrays(b, exact=True)
    assert len(a_keys) == n and np.array_equal(a_keys, b_keys) and np.array_equal(a_keys, keys)


def _weakly_stable_sample(index_a, index_b, vectors, a_keys, b_keys, men, width, expansion):
    """Blocking pairs among a sample of men of a join of an index with a snapshot of its own image (keys = rows): their lists from the
    device's own search, the women's view by the same distances (the metric is symmetric bit for bit, tests/test_join_model.py)."""
    found = index_b.search(vectors[men], width, expansion=expansion)
    matching = dict(zip(a_keys.tolist(), b_keys.tolist()))
    husband_of = {w: m for m, w in matching.items()}
    blocking = []
    for row, man in enumerate(men.tolist()):
        own = matching.get(man)
        entries = list(zip(found.keys[row, :int(found.counts[row])].tolist(), found.distances[row, :int(found.counts[row])].tolist()))
        own_d = next((d for w, d in entries if w == own), np.inf) if own is not None else np.inf
        for woman, d in entries:
            if not d < own_d:
                break
            husband = husband_of.get(woman)
            if husband is None:
                blocking.append((man, woman))
                continue
            her_view = index_b.distances(vectors[[woman]], np.array([[husband, man]], dtype=np.uint32))[0]
            if her_view[1] < her_view[0]:
                blocking.append((man, woman))
    return blocking


def test_join_through_every_surface(tmp_path):
    """Python, the drop-in table's `join` entry and the C++ class surface called the way cpp/bench.cpp:412-445 calls it (free
    `join` with raw key arrays, then the member `join` with `unordered_map`s) give the same matching."""
    import ctypes as C
    import os
    import subprocess

    from usearch_amd import Index
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    binary = build_join_surface(tmp_path)
    men_path, women_path = str(tmp_path / "men.usearch"), str(tmp_path / "women.usearch")
    out = subprocess.run([binary, "run", men_path, women_path], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    from_cpp = {int(m): int(w) for _, m, w in (line.split() for line in out.stdout.splitlines() if line.startswith("pair "))}
    assert from_cpp
    # Python over snapshots of the two saved images; P = executor.size() = 4, as the C++ program asks
    men, women = Index.restore(men_path), Index.restore(women_path)
    assert men.join(women, max_proposals=4) == from_cpp
    # the drop-in table entry over the two indexes loaded by the drop-in itself
    L = C.CDLL(os.path.join(root, "usearch_amd", "lib", "libusearch_c.so"))
    err = C.c_char_p()
    L.usearch_init.restype = C.c_void_p
    L.usearch_init.argtypes = [C.c_void_p, C.POINTER(C.c_char_p)]
    L.usearch_load.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_char_p)]
    L.usearch_free.argtypes = [C.c_void_p, C.POINTER(C.c_char_p)]
    L.usearch_remove.restype = C.c_size_t
    L.usearch_remove.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_char_p)]
    L.usearch_amd_c_api.restype = C.POINTER(C.c_void_p)
    table = L.usearch_amd_c_api()
    assert table[0] == 52, "the table's entry count"
    join = C.CFUNCTYPE(C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_bool, C.c_size_t, C.c_void_p, C.c_void_p,
                       C.c_size_t, C.c_void_p, C.POINTER(C.c_char_p))(table[52])
    handles = []
    for path in (men_path, women_path):
        handle = L.usearch_init(None, C.byref(err))
        L.usearch_load(handle, path.encode(), C.byref(err))
        assert not err.value, err.value
        handles.append(handle)
    a_keys, b_keys = np.zeros(1500, dtype=np.uint64), np.zeros(1500, dtype=np.uint64)
    stats = np.zeros(4, dtype=np.uint64)
    pairs = join(handles[0], handles[1], 4, 64, False, 1, a_keys.ctypes.data, b_keys.ctypes.data, 1500, stats.ctypes.data, C.byref(err))
    assert not err.value, err.value
    assert dict(zip(a_keys[:pairs].tolist(), b_keys[:pairs].tolist())) == from_cpp and stats[0] == pairs
    pairs = join(handles[0], handles[0], 4, 64, False, 1, a_keys.ctypes.data, b_keys.ctypes.data, 1500, None, C.byref(err))
    assert pairs == 0 and b"Can't join with itself" in err.value
    # members removed through the drop-in never appear
    err = C.c_char_p()
    removed_men, removed_women = list(range(0, 1500, 3)), list(range(1, 1800, 4))
    for handle, keys in zip(handles, (removed_men, removed_women)):
        for key in keys:
            assert L.usearch_remove(handle, key, C.byref(err)) == 1
    pairs = join(handles[0], handles[1], 4, 64, False, 1, a_keys.ctypes.data, b_keys.ctypes.data, 1500, None, C.byref(err))
    assert not err.value, err.value
    assert pairs > 0
    assert not np.isin(a_keys[:pairs], removed_men).any() and not np.isin(b_keys[:pairs], removed_women).any()
    assert not (a_keys[:pairs] == np.uint64(2**64 - 1)).any() and not (b_keys[:pairs] == np.uint64(2**64 - 1)).any()
    for handle in handles:
        L.usearch_free(handle, C.byref(err))

